"""Global-norm gradient clipping inside the fused AdamW step, on the GPU: the two norm kernels through the C ABI (kan_grad_sqnorm_chunks,
kan_grad_norm_finish), the two _clip step entry points, FusedAdamW(max_grad_norm=...) as an optimizer against clip_grad_norm_ +
torch.optim.AdamW in fp64, the recorded step against the same steps run eagerly, and the off path (max_grad_norm=None) against an optimizer
built without the keyword.

Tolerances.  seg_sq: 1e-12 relative in double -- a double sum of at most 1e5 exact squares errs below 1e5 x 2^-53 = 1.1e-11 in the worst case of
a serial sum and far less in the tree the kernel uses.  norm and scale: ONE float32 ulp of the fp64 expression rounded to float32 -- the kernel
forms both in double and rounds once, and a tie can fall either way.  p, m, v of a step: adamw_cells.judge, max(FLOOR = 2e-6, 4 x the fp32 CPU
execution's own error, measured live), nothing masked; trajectories: the rule tests/test_optim.py applies to trajectories (restated in
_judge_trajectory).  Everything recorded is compared with torch.equal (the moments of the PReLU slopes excepted, as in
tests/test_gpu_optim_capturable.py: their gradients are float-atomic sums)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import adamw_cells as A
from test_gpu_optim_capturable import PRESET, SEGS, SLOPE_GRAD_NOISE, _cell_inputs

pytestmark = pytest.mark.gpu

SENT_F = 0x7FA5A5A5                                                        # NaN patterns no kernel writes
SENT_D = 0x7FF5A5A5A5A5A5A5
CHUNK = 8192
SEGS_C8 = [(996, 0), (997, 0), (998, 0), (999, 1), (1000, 0), (1001, 0), (1002, None), (1003, 0), (1004, 0)]      # chunk_elems = 8: 125 or 126 chunks each


def _p(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(xs, dt):
    return torch.tensor(xs, dtype=dt, device="cuda")


def _ulps(a, b):
    """Distance in float32 ulps of two finite float32 values of the same sign."""
    a, b = np.float32(a), np.float32(b)
    assert np.isfinite(a) and np.isfinite(b), (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


class _Grads:
    """The gradient buffers of one segment set -- one allocation per segment, the view `offset` floats past a 16-byte boundary -- and the device
    tables the kernels read: seg_grad, seg_n, the chunk table, seg_first_chunk."""

    def __init__(self, segs, chunk, values):
        self.segs, self.chunk, self.stores, addr = segs, chunk, [], []
        chunk_seg, chunk_start, first = [], [], [0]
        for i, ((n, goff), val) in enumerate(zip(segs, values)):
            for s0 in range(0, n, chunk):
                chunk_seg.append(i); chunk_start.append(s0)
            first.append(len(chunk_seg))
            if goff is None:
                addr.append(0)
                continue
            self.stores.append(torch.full((n + goff + 1,), 7.0, device="cuda"))
            view = self.stores[-1][goff:goff + n]
            view.copy_(val)
            assert view.data_ptr() & 15 == 4 * goff
            addr.append(view.data_ptr())
        self.n_chunks, self.n_seg, self.first = len(chunk_seg), len(segs), first
        self.tab = dict(seg_grad=_dev(addr, torch.int64), seg_n=_dev([n for n, _ in segs], torch.int32), chunk_seg=_dev(chunk_seg, torch.int32),
                        chunk_start=_dev(chunk_start, torch.int32), seg_first_chunk=_dev(first, torch.int32))
        self.before = {k: t.clone() for k, t in self.tab.items()}
        self.stores0 = [s.clone() for s in self.stores]

    def untouched(self):
        bad = [f"table {k} was written" for k, t in self.tab.items() if not torch.equal(t, self.before[k])]
        if not all(torch.equal(s.view(torch.int32), s0.view(torch.int32)) for s, s0 in zip(self.stores, self.stores0)):
            bad.append("a gradient buffer was written")
        return bad


class _Stats:
    """partial, seg_sq and out (norm, scale), each between eight sentinel words, and max_norm in a tensor of its own."""

    def __init__(self, grads):
        self.g = grads
        self.partial_buf = torch.full((grads.n_chunks + 16,), SENT_D, dtype=torch.int64, device="cuda")
        self.seg_sq_buf = torch.full((grads.n_seg + 16,), SENT_D, dtype=torch.int64, device="cuda")
        self.out_buf = torch.full((2 + 16,), SENT_F, dtype=torch.int32, device="cuda")
        self.partial = self.partial_buf.view(torch.float64)[8:8 + grads.n_chunks]
        self.seg_sq = self.seg_sq_buf.view(torch.float64)[8:8 + grads.n_seg]
        self.out = self.out_buf.view(torch.float32)[8:10]
        self.max_norm = torch.zeros(1, device="cuda")

    def chunks(self, lib):
        from convkan_amd import _lib as L
        t = self.g.tab
        L.check(lib.kan_grad_sqnorm_chunks(_p(t["seg_grad"]), _p(t["seg_n"]), _p(t["chunk_seg"]), _p(t["chunk_start"]), self.g.n_chunks, self.g.chunk,
                                           _p(self.partial), _stream()), "kan_grad_sqnorm_chunks")

    def finish(self, lib, max_norm):
        from convkan_amd import _lib as L
        self.max_norm.fill_(max_norm)
        L.check(lib.kan_grad_norm_finish(_p(self.partial), _p(self.g.tab["seg_first_chunk"]), self.g.n_seg, _p(self.max_norm), _p(self.seg_sq),
                                         _p(self.out), _stream()), "kan_grad_norm_finish")
        torch.cuda.synchronize()
        norm, scale = (np.float32(x) for x in self.out.tolist())
        return norm, scale

    def sentinels(self):
        bad = []
        for name, buf, sent in (("partial", self.partial_buf, SENT_D), ("seg_sq", self.seg_sq_buf, SENT_D), ("out", self.out_buf, SENT_F)):
            if not (bool((buf[:8] == sent).all()) and bool((buf[-8:] == sent).all())):
                bad.append(f"memory next to {name} was written")
        return bad


def _values(segs, seed):
    """One fp32 gradient per segment; the magnitude grows from 1e-3 (first segment) to 1e3 (last)."""
    gen = torch.Generator().manual_seed(seed)
    k = len(segs) - 1
    return [(torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (-3.0 + 6.0 * i / k)).float() for i, (n, _) in enumerate(segs)]


def _fp64_scale(total_sq, max_norm):
    """torch's clip_coef = max_norm / (total_norm + 1e-6), clamped to 1, in fp64, rounded to float32 once.  max_norm: the float32 the device holds."""
    with np.errstate(all="ignore"):
        return np.float32(min(1.0, float(np.float64(np.float32(max_norm)) / (np.sqrt(np.float64(total_sq)) + 1e-6))))


# ------------------------------------------------------------------------------------------------ 1. norm cells through the C ABI
@pytest.mark.parametrize("name,segs,chunk", [("c8192", SEGS, CHUNK), ("c8", SEGS_C8, 8)])
def test_norm_cells_vs_fp64(name, segs, chunk, gpu_lib):
    vals = _values(segs, 500 + chunk)
    grads = _Grads(segs, chunk, vals)
    if chunk == 8:
        assert all(b - a > 64 for a, b in zip(grads.first, grads.first[1:])) and grads.n_seg > 4       # the lane stride wraps; more segments than waves
    ref_sq = [0.0 if goff is None else float((v.double() ** 2).sum()) for (n, goff), v in zip(segs, vals)]
    total = 0.0
    for x in ref_sq:
        total += x
    ref_norm = np.float32(math.sqrt(total))
    st = _Stats(grads)
    st.chunks(gpu_lib)
    bad = []
    runs = {}
    for tag, mx in (("2 x norm", np.float32(2.0 * float(ref_norm))), ("norm / 2", np.float32(0.5 * float(ref_norm))), ("1e-3", np.float32(1e-3)),
                    ("0", np.float32(0.0)), ("inf", np.float32(np.inf))):
        norm, scale = st.finish(gpu_lib, float(mx))
        runs[tag] = (norm, scale)
        want = _fp64_scale(total, mx)
        print(f"[clip cells] {name} max_norm {tag}: norm {norm!r} (fp64 {ref_norm!r}), scale {scale!r} (fp64 {want!r})")
        if _ulps(norm, ref_norm) > 1:
            bad.append(f"max_norm {tag}: norm {norm!r} is {_ulps(norm, ref_norm)} ulps from {ref_norm!r}")
        if _ulps(scale, want) > 1:
            bad.append(f"max_norm {tag}: scale {scale!r} is {_ulps(scale, want)} ulps from {want!r}")
        if tag in ("2 x norm", "inf") and float(scale) != 1.0:
            bad.append(f"max_norm {tag}: scale {scale!r} is not exactly 1")
    assert float(runs["0"][1]) == 0.0 and 0.4 < float(runs["norm / 2"][1]) < 0.6
    got_sq = st.seg_sq.cpu().tolist()
    partial = st.partial.cpu()
    for i, ((n, goff), want) in enumerate(zip(segs, ref_sq)):
        if goff is None:
            if got_sq[i] != 0.0 or bool((partial[grads.first[i]:grads.first[i + 1]] != 0.0).any()):
                bad.append(f"segment {i} has a null gradient: seg_sq {got_sq[i]!r}, partials not all exactly 0")
        elif not abs(got_sq[i] - want) <= 1e-12 * want:
            bad.append(f"segment {i} ({n} elements): seg_sq {got_sq[i]!r} vs fp64 {want!r} (relative {abs(got_sq[i] - want) / want:.2e})")
    # two launches, identical bits
    again = _Stats(grads)
    again.chunks(gpu_lib)
    n2, s2 = again.finish(gpu_lib, float("inf"))
    if not (torch.equal(again.partial.view(torch.int64), st.partial.view(torch.int64)) and torch.equal(again.seg_sq.view(torch.int64), st.seg_sq.view(torch.int64))
            and n2.view(np.int32) == runs["inf"][0].view(np.int32) and s2.view(np.int32) == runs["inf"][1].view(np.int32)):
        bad.append("a second launch over the same gradients gave other bits")
    bad += st.sentinels() + again.sentinels() + grads.untouched()
    assert not bad, f"{name}:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("poison", ["inf", "nan"])
def test_norm_cells_non_finite_gradients_follow_torch(poison, gpu_lib):
    """One inf (one NaN) element in the 8192-element segment: norm and scale are what clip_grad_norm_'s expression gives on the CPU."""
    vals = _values(SEGS, 777)
    vals[5] = vals[5].clone()
    vals[5][4097] = float(poison)
    grads = _Grads(SEGS, CHUNK, vals)
    st = _Stats(grads)
    st.chunks(gpu_lib)
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or a == b
    bad = []
    for mx in (1.0, 0.0, float("inf")):
        ps = [nn.Parameter(torch.zeros_like(v)) for (n, goff), v in zip(SEGS, vals) if goff is not None]
        for p, v in zip(ps, [v for (n, goff), v in zip(SEGS, vals) if goff is not None]):
            p.grad = v.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, mx, foreach=False)
        coef = torch.clamp(mx / (total + 1e-6), max=1.0)
        norm, scale = st.finish(gpu_lib, mx)
        print(f"[clip cells] one {poison}, max_norm {mx}: norm {norm!r} scale {scale!r}; torch {float(total)!r} {float(coef)!r}")
        if not (same(float(norm), float(total)) and same(float(scale), float(coef))):
            bad.append(f"max_norm {mx}: norm {norm!r} scale {scale!r}, torch gives {float(total)!r} {float(coef)!r}")
    bad += st.sentinels() + grads.untouched()
    assert not bad, "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------ 2. step cells
def _step_cells(lib, entry, case, inp, lay, grads, scale_dev):
    """One clipped step over the row's segments by `entry` ("classic": kan_adamw_step_segments_clip with the bias table of the per-segment step
    counts; "dev": kan_adamw_advance + kan_adamw_step_segments_dev_clip from PRESET).  Returns (dense p / m / v, findings)."""
    from convkan_amd import _lib as L
    nb = lay["n_blk"]
    pos = torch.cat([torch.arange(o, o + n) for o, n in zip(lay["seg_off"], lay["seg_n"])]).cuda()
    gap = torch.ones(nb, dtype=torch.bool, device="cuda")
    gap[pos] = False
    blk = {k: torch.full((nb + 128,), SENT_F, dtype=torch.int32, device="cuda").view(torch.float32) for k in "pmv"}
    for k in "pmv":
        blk[k][64:64 + nb][pos] = inp[k].cuda()
    seg_off = _dev(lay["seg_off"], torch.int64)
    lr, (b1, b2), eps, wd = A.HYPER[case["hyper"]]
    views = [_p(blk[k][64:64 + nb]) for k in "pmv"]
    t = grads.tab
    tabs = [_p(t["seg_grad"]), _p(seg_off), _p(t["seg_n"]), _p(t["chunk_seg"]), _p(t["chunk_start"])]
    bad = []
    if entry == "dev":
        seg_step, lr_dev = _dev(PRESET, torch.int32), torch.full((1,), lr, dtype=torch.float64, device="cuda")
        L.check(lib.kan_adamw_advance(_p(seg_step), _p(t["seg_grad"]), grads.n_seg, _stream()), "kan_adamw_advance")
        L.check(lib.kan_adamw_step_segments_dev_clip(*views, *tabs, _p(lr_dev), _p(seg_step), grads.n_chunks, CHUNK, b1, b2, eps, wd, scale_dev, _stream()),
                "kan_adamw_step_segments_dev_clip")
        torch.cuda.synchronize()
        if seg_step.tolist() != case["bias"]:
            bad.append(f"seg_step {seg_step.tolist()} != {case['bias']}")
    else:
        bias = _dev(A.bias_table(case["hyper"], case["bias"]), torch.float32)
        L.check(lib.kan_adamw_step_segments_clip(*views, *tabs, _p(bias), grads.n_chunks, CHUNK, lr, b1, b2, eps, wd, max(case["bias"]), scale_dev, _stream()),
                "kan_adamw_step_segments_clip")
        torch.cuda.synchronize()
    out = {}
    for k in "pmv":
        raw = blk[k].view(torch.int32)
        if not (bool((raw[:64] == SENT_F).all()) and bool((raw[-64:] == SENT_F).all())):
            bad.append(f"{k}: memory next to the block was written")
        if not bool((raw[64:64 + nb][gap] == SENT_F).all()):
            bad.append(f"{k}: elements in the gaps between segments were written")
        out[k] = blk[k][64:64 + nb][pos].cpu()
    return out, bad


@pytest.mark.parametrize("hyper", ["default", "all", "b00"])
def test_clip_step_cells_vs_fp64(hyper, gpu_lib):
    """Both _clip entry points over SEGS, the scale left in device memory by a finish launch in front of them (max_norm = 0.37 x the fp64 norm of the
    row's gradients: a scale near 0.37); judged against adamw_cells.reference with gscale = that scale read back."""
    steps = [s + (goff is not None) for s, (_, goff) in zip(PRESET, SEGS)]
    case = dict(kind="seg", chunk=CHUNK, segs=SEGS, hyper=hyper, step=max(steps), gscale=1.0, state="rand", bias=steps, bucket=False, flatten=False, mask=None)
    lay = A.layout(case)
    inp = _cell_inputs(case, 5100 + list(A.HYPER).index(hyper))
    per_seg = [inp["g"][lay["elem_off"][i]:lay["elem_off"][i] + n] for i, (n, _) in enumerate(SEGS)]
    grads = _Grads(SEGS, CHUNK, per_seg)
    assert grads.tab["chunk_seg"].tolist() == lay["chunk_seg"] and grads.tab["chunk_start"].tolist() == lay["chunk_start"]
    total = sum(float((g.double() ** 2).sum()) for (n, goff), g in zip(SEGS, per_seg) if goff is not None)
    st = _Stats(grads)
    st.chunks(gpu_lib)
    norm, scale = st.finish(gpu_lib, float(np.float32(0.37 * math.sqrt(total))))
    assert _ulps(norm, np.float32(math.sqrt(total))) <= 1 and 0.36 < float(scale) < 0.38
    case["gscale"] = float(scale)
    r64, r32 = A.reference(case, inp, torch.float64), A.reference(case, inp, torch.float32)
    bad = []
    for entry in ("classic", "dev"):
        got, wrong = _step_cells(gpu_lib, entry, case, inp, lay, grads, _p(st.out, 4))
        lines, judged = A.judge(case, inp, got, r64, r32)
        print(f"[clip step cells] {hyper} {entry} (scale {float(scale)!r}): " + "; ".join(lines))
        bad += [f"{entry}: {b}" for b in wrong + judged]
        for i, (n, goff) in enumerate(SEGS):
            sl = slice(lay["elem_off"][i], lay["elem_off"][i] + n)
            if goff is None and not all(torch.equal(got[k][sl].view(torch.int32), inp[k][sl].view(torch.int32)) for k in "pmv"):
                bad.append(f"{entry}: segment {i} has a null gradient and changed")
    bad += st.sentinels() + grads.untouched()
    assert not bad, f"{hyper}:\n  " + "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------ 3. optimizer trajectory
def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 5), nn.PReLU(), nn.Linear(5, 3, bias=False))


def _judge_trajectory(tag, p0, got, r64, r32):
    """tests/test_optim.py's rule.  got / r64 / r32: (p, exp_avg, exp_avg_sq).  Returns the failures."""
    d = lambda t: t.detach().double().cpu().reshape(-1)
    zero, bad, line = d(p0) == 0, [], []

    def errs(r):
        e = {}
        for name, sel in (("p(from 0)", zero), ("p(rest)", ~zero)):
            if bool(sel.any()):
                e[name] = float(((d(r[0]) - d(r64[0]))[sel].abs() / (d(r64[0])[sel].abs().max() + 1e-300)).max())
        e["m"] = float(((d(r[1]) - d(r64[1])).abs() / (d(r64[1]).abs().max() + 1e-300)).max())
        e["v"] = float(((d(r[2]) - d(r64[2])).abs() / (d(r64[2]) + 1e-300)).max())
        return e
    err, noise = errs(got), errs(r32)
    for name, e in err.items():
        tol = max(A.FLOOR, 4.0 * noise[name])
        line.append(f"{name} {e:.1e} (tol {tol:.1e}, fp32 reference {noise[name]:.1e})")
        if not e <= tol:
            bad.append(f"{tag} {name}: error {e:.3e} > {tol:.3e} (fp32 reference {noise[name]:.3e})")
    print(f"[clip trajectory] {tag}: " + "; ".join(line))
    return bad


def _state(opt, i, like):
    st = opt.state_dict()["state"]
    if i not in st:
        return torch.zeros_like(like), torch.zeros_like(like), 0
    return st[i]["exp_avg"], st[i]["exp_avg_sq"], int(st[i]["step"])


TRAJ_MAX_NORM = 1.0
TRAJ_MULT = (1e-2, 1e2, 1e-2, 1e2, 1e-2, 1e2)                            # loss multipliers: the gradient norm alternates between small and large
TRAJ_GROUPS = (dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.1))


def fp64_trajectory():
    """The fp64 CPU reference: the small net under clip_grad_norm_(TRAJ_MAX_NORM) + torch.optim.AdamW in two groups, six steps, the loss of step k
    multiplied by TRAJ_MULT[k]; the PReLU slope has no gradient at the first step.  Every gradient is rounded to fp32 before it is clipped and
    consumed, so that the optimizers under test can be fed the very same values.  Returns (start values, per step the fp32 gradients, per step
    the fp64 norm and scale, the reference's parameters and optimizer)."""
    net = _net().double()
    ps = list(net.parameters())
    p0 = [p.detach().clone().float() for p in ps]
    with torch.no_grad():
        for p, v in zip(ps, p0):
            p.copy_(v.double())
    opt = torch.optim.AdamW([dict(params=ps[:2], **TRAJ_GROUPS[0]), dict(params=ps[2:], **TRAJ_GROUPS[1])], foreach=False)
    gen = torch.Generator().manual_seed(77)
    fed, stats = [], []
    for it, mult in enumerate(TRAJ_MULT):
        x, t = torch.randn(16, 7, generator=gen, dtype=torch.float64), torch.randint(0, 3, (16,), generator=gen)
        opt.zero_grad()
        (mult * nn.functional.cross_entropy(net(x), t)).backward()
        if it == 0:
            ps[2].grad = None
        step = [None if p.grad is None else p.grad.float() for p in ps]
        for p, g in zip(ps, step):
            if g is not None:
                p.grad = g.double()
        total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in step if g is not None))
        stats.append((total, min(1.0, TRAJ_MAX_NORM / (total + 1e-6)), [0.0 if g is None else math.sqrt(float((g.double() ** 2).sum())) for g in step]))
        torch.nn.utils.clip_grad_norm_(ps, TRAJ_MAX_NORM, foreach=False)
        opt.step()
        fed.append(step)
    return p0, fed, stats, ps, opt


def trajectory_condition(stats):
    scales = [s for _, s, _ in stats]
    return sum(s < 0.9 for s in scales) >= 2 and sum(s == 1.0 for s in scales) >= 2


@pytest.mark.parametrize("capturable", [False, True])
def test_trajectory_vs_clip_grad_norm_and_torch_adamw_fp64(capturable, gpu_lib):
    from convkan_amd import FusedAdamW
    p0, fed, stats, r64, opt64 = fp64_trajectory()
    assert trajectory_condition(stats), [s for _, s, _ in stats]           # from the fp64 reference alone: clipped at >= 2 steps, untouched at >= 2
    r32 = [nn.Parameter(v.clone()) for v in p0]
    opt32 = torch.optim.AdamW([dict(params=r32[:2], **TRAJ_GROUPS[0]), dict(params=r32[2:], **TRAJ_GROUPS[1])], foreach=False)
    dev = [nn.Parameter(v.clone().cuda()) for v in p0]
    opt = FusedAdamW([dict(params=dev[:2], **TRAJ_GROUPS[0]), dict(params=dev[2:], **TRAJ_GROUPS[1])], capturable=capturable, max_grad_norm=TRAJ_MAX_NORM)
    bad = []
    for it, (step, (total, scale, per)) in enumerate(zip(fed, stats)):
        for p, g in zip(r32, step):
            p.grad = None if g is None else g.clone()
        torch.nn.utils.clip_grad_norm_(r32, TRAJ_MAX_NORM, foreach=False)
        opt32.step()
        for p, g in zip(dev, step):
            p.grad = None if g is None else g.cuda()
        kept = [None if p.grad is None else p.grad.clone() for p in dev]
        opt.step()
        for i, (p, k) in enumerate(zip(dev, kept)):
            if k is not None and not torch.equal(p.grad.view(torch.int32), k.view(torch.int32)):
                bad.append(f"step {it}: the gradient of parameter {i} was modified")
        norm, got_scale, norms = np.float32(float(opt.grad_norm)), np.float32(float(opt.clip_scale)), opt.grad_norms().tolist()
        print(f"[clip trajectory] step {it}: norm {norm!r} (fp64 {total!r}), scale {got_scale!r} (fp64 {scale!r})")
        if _ulps(norm, np.float32(total)) > 1 or _ulps(got_scale, np.float32(scale)) > 1:
            bad.append(f"step {it}: norm {norm!r} / scale {got_scale!r} against fp64 {total!r} / {scale!r}")
        if scale == 1.0 and float(got_scale) != 1.0:
            bad.append(f"step {it}: scale {got_scale!r} is not exactly 1")
        for i, (a, b) in enumerate(zip(norms, per)):
            if (b == 0.0 and a != 0.0) or (b != 0.0 and _ulps(a, np.float32(b)) > 1):
                bad.append(f"step {it}: grad_norms()[{i}] {a!r} against fp64 {b!r}")
    assert opt.grad_norm.is_cuda and opt.clip_scale.is_cuda and opt.grad_norms().is_cuda
    for i in range(4):
        bad += _judge_trajectory(f"param {i}", p0[i], (dev[i], *_state(opt, i, dev[i])[:2]), (r64[i], *_state(opt64, i, r64[i])[:2]),
                                 (r32[i], *_state(opt32, i, r32[i])[:2]))
        assert _state(opt, i, dev[i])[2] == _state(opt64, i, r64[i])[2] == (5 if i == 2 else 6)
    assert not bad, "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------ 4. recorded step == eager step
def test_recorded_clipping_step_equals_eager_steps_bitwise(gpu_lib):
    """Four steps of KAN-VGG11 at bs 4 with max_grad_norm = 1e-3 (far below the gradient norm of a fresh net: every step is clipped), eager
    train_step against GraphedStep(optimizer=...) from a deep copy: losses, parameters, exp_avg / exp_avg_sq, the step counts, grad_norm and
    clip_scale are torch.equal.  Then max_grad_norm is set to 1e6 on both (no step is clipped any more) and a fifth step follows: equal again, the
    scale exactly 1, and the graph object is the one recorded at the start.

    As in tests/test_gpu_optim_capturable.py, the moments of the eight PReLU slopes are bounded instead of compared bit for bit: their gradients are
    float-atomic sums that differ between two eager runs already; with a scale <= 1 in front of them the bounds of that test hold unchanged.  The
    same noise reaches the global norm at about 1e-10 relative, far below float32 resolution."""
    import convkan_amd as K
    from convkan_amd.models import vggkan
    torch.manual_seed(7)
    base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", dropout_linear=0.0).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(4, 3, 32, 32, device="cuda", generator=g), torch.randint(0, 10, (4,), device="cuda", generator=g)) for _ in range(5)]
    out, gmax = {}, {}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base)
        slopes = {i for i, (n, p) in enumerate(model.named_parameters()) if isinstance(model.get_submodule(n.rsplit(".", 1)[0]), nn.PReLU)}
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True, max_grad_norm=1e-3)
        params = opt._flat[0]["params"]
        step = K.GraphedStep(model, *batches[0], optimizer=opt) if mode == "graph" else None
        graph = step.graph if step is not None else None
        seen = []
        for it, (d, t) in enumerate(batches):
            if it == 4:
                opt.max_grad_norm = 1e6
            loss = (step(d, t) if step is not None else K.train_step(model, d, t, opt)).clone()
            if mode == "eager":
                for i in slopes:
                    gmax[i] = torch.maximum(gmax.get(i, torch.zeros((), device="cuda")), params[i].grad.abs().max())
            flat = opt._flat[0]
            seen.append((loss, [tuple(x.clone() for x in v) for v in flat["views"]], flat["tab"]["seg_step"].clone(), opt.grad_norm.clone(),
                         opt.clip_scale.clone()))
        torch.cuda.synchronize()
        assert step is None or step.graph is graph                         # nothing was recorded again
        out[mode] = seen
    bad = []
    for it, (e, r) in enumerate(zip(out["eager"], out["graph"])):
        for name, a, b in (("loss", e[0], r[0]), ("seg_step", e[2], r[2]), ("grad_norm", e[3], r[3]), ("clip_scale", e[4], r[4])):
            if not torch.equal(a, b):
                bad.append(f"step {it}: {name} differs: eager {a.tolist()} recorded {b.tolist()}")
        assert e[2].tolist() == [it + 1] * len(e[1])
        print(f"[clip graph] step {it}: norm {float(e[3])!r} scale {float(e[4])!r}")
        assert (float(e[4]) < 0.5) if it < 4 else (float(e[4]) == 1.0), (it, float(e[4]))
        for i, (a, b) in enumerate(zip(e[1], r[1])):
            if not torch.equal(a[0], b[0]):
                bad.append(f"step {it}, parameter {i}: {int((a[0] != b[0]).sum())} elements differ")
            for row, name, width in ((1, "exp_avg", 1.0), (2, "exp_avg_sq", 2.0)):
                if i in slopes:
                    d, tol = float((a[row].double() - b[row].double()).abs().max()), width * SLOPE_GRAD_NOISE * float(gmax[i]) ** row
                    if not d <= tol:
                        bad.append(f"step {it}, {name} of slope {i}: {d:.3e} > {tol:.3e}")
                elif not torch.equal(a[row], b[row]):
                    bad.append(f"step {it}, {name} of parameter {i}: {int((a[row] != b[row]).sum())} elements differ")
    assert not bad, "\n  ".join(bad[:40])


def test_recording_with_a_stale_max_grad_norm_raises(gpu_lib):
    """Like lr: a value the device copy does not hold cannot be uploaded while the stream is capturing."""
    import convkan_amd as K
    from convkan_amd._lib import KanConvError
    model = _net().cuda().train()
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, capturable=True, max_grad_norm=1.0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    d, t = torch.randn(8, 7, device="cuda", generator=gen), torch.randint(0, 3, (8,), device="cuda", generator=gen)
    K.train_step(model, d, t, opt)                       # lr and max_grad_norm are on the device now
    before = opt._flat[0]["block"].clone()
    opt.max_grad_norm = 0.5                              # ... and the device copy is stale now
    scratch = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(KanConvError, match="sync_hyper"):
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt._flat[0]["block"], before) and opt._flat[0]["tab"]["seg_step"].tolist() == [1, 1, 1, 1]
    opt.sync_hyper()
    assert float(opt._clip["out"][2]) == 0.5


# ------------------------------------------------------------------------------------------------ 5. off path
class _Counting:
    """The library handle with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("capturable", [False, True])
def test_off_path_is_the_plain_step(capturable, gpu_lib, monkeypatch):
    """max_grad_norm=None against an optimizer built without the keyword: three steps over two groups, the same calls into the library and
    torch.equal blocks.  (With clipping on the same steps add one chunk launch per group and one finish per step.)"""
    from convkan_amd import FusedAdamW
    from convkan_amd import _lib as L
    p0, fed, _, _, _ = fp64_trajectory()
    results = {}
    for tag, kw in (("plain", {}), ("off", dict(max_grad_norm=None)), ("on", dict(max_grad_norm=TRAJ_MAX_NORM))):
        ps = [nn.Parameter(v.clone().cuda()) for v in p0]
        opt = FusedAdamW([dict(params=ps[:2], **TRAJ_GROUPS[0]), dict(params=ps[2:], **TRAJ_GROUPS[1])], capturable=capturable, **kw)
        counting = _Counting(gpu_lib)
        monkeypatch.setattr(L, "load", lambda: counting)
        for step in fed[:3]:
            for p, g in zip(ps, step):
                p.grad = None if g is None else g.cuda()
            opt.step()
        monkeypatch.undo()
        torch.cuda.synchronize()
        counting.calls.pop("kan_last_error", None)
        results[tag] = (dict(counting.calls), [f["block"].clone() for f in opt._flat], [f["tab"]["seg_step"].clone() for f in opt._flat])
    plain, off, on = results["plain"], results["off"], results["on"]
    print(f"[clip off path] capturable={capturable}: plain {plain[0]}, on {on[0]}")
    assert off[0] == plain[0] and sum(plain[0].values()) == (12 if capturable else 6)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(off[1], plain[1]))
    assert all(torch.equal(a, b) for a, b in zip(off[2], plain[2]))
    assert sum(on[0].values()) == sum(plain[0].values()) + 3 * (2 + 1)
    assert on[0]["kan_grad_sqnorm_chunks"] == 6 and on[0]["kan_grad_norm_finish"] == 3
    assert not any(n.endswith("_clip") for n in plain[0]) and not any(n in on[0] for n in ("kan_adamw_step_segments", "kan_adamw_step_segments_dev"))
