"""The capturable AdamW step on the GPU: the device-formed scalars (kan_adamw_dev_args), the kernels behind kan_adamw_advance +
kan_adamw_step_segments_dev, kan_set_u64_table, FusedAdamW(capturable=True) as an optimizer (trajectory, resume in every direction), and
train.GraphedStep(optimizer=...) / the graphed drivers against the same steps run eagerly, bit for bit.

Tolerances.  The nine floats: one float32 ulp -- device pow and host pow may differ in the last bit of a double (1e-15 relative, three digits
lost at most in 1 - beta^step at the tested values) in front of a rounding whose half-spacing is 6e-8; they cannot differ by more.  p, m, v:
adamw_cells.judge, max(FLOOR = 2e-6, 4 x the fp32 CPU execution's own error, measured live), nothing masked; trajectories: the same rule as
tests/test_optim.py applies it to trajectories (restated in _judge_trajectory).  Everything recorded is compared with torch.equal (the moments of the PReLU slopes
excepted, whose gradients are float-atomic sums: see test 6)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import adamw_cells as A

pytestmark = pytest.mark.gpu

FIELDS = ("decay", "w1", "b1", "b2", "w2", "gscale", "inv_bc2_sqrt", "eps", "neg_step")         # AdamArgs order (csrc/kanconv.hip)
SENT_F = 0x7FA5A5A5                                                                              # NaN pattern no kernel writes
CHUNK = 8192


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_args(hyper, step, gscale=1.0):
    """adam_args() of csrc/kanconv.hip in numpy float64, every result rounded to float32 once."""
    lr, (b1, b2), eps, wd = (np.float64(x) if not isinstance(x, tuple) else tuple(np.float64(y) for y in x) for x in hyper)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        bc1, bc2 = one - np.power(b1, np.float64(step)), one - np.power(b2, np.float64(step))
        vals = (one - lr * wd, one - b1, b1, b2, one - b2, np.float64(gscale), one / np.sqrt(bc2), eps, -lr / bc1)
        return np.array([np.float32(x) for x in vals], dtype=np.float32)


@functools.lru_cache(maxsize=1)
def _scalar_table():
    """{(hyper name, step): (device floats, host floats)} for HYPER x STEPS -- computed once, shared by tests 1 and 2."""
    from convkan_amd import _lib as L
    lib = L.load()
    out = {}
    lr_dev, st_dev, res = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(9, device="cuda")
    for name, hyper in A.HYPER.items():
        lr, (b1, b2), eps, wd = hyper
        for step in A.STEPS:
            lr_dev.fill_(lr); st_dev.fill_(step); res.fill_(float("nan"))
            L.check(lib.kan_adamw_dev_args(_p(lr_dev), _p(st_dev), b1, b2, eps, wd, 1.0, _p(res), _stream()), "kan_adamw_dev_args")
            out[(name, step)] = (res.cpu().numpy().copy(), _host_args(hyper, step))
    return out


# ------------------------------------------------------------------------------------------------ 1. scalars
def test_device_scalars_within_one_ulp_of_the_host(gpu_lib):
    table, bad, off = _scalar_table(), [], 0
    for (name, step), (dev, host) in table.items():
        assert np.isfinite(dev).all() and np.isfinite(host).all(), (name, step, dev, host)
        d = np.abs(dev.view(np.int32).astype(np.int64) - host.view(np.int32).astype(np.int64))         # same sign, finite: distance in ulps
        off += int((d != 0).sum())
        for i in np.nonzero(d > 1)[0]:
            bad.append(f"{name} step {step}: {FIELDS[i]} device {dev[i]!r} host {host[i]!r} ({d[i]} ulps)")
    print(f"[capturable scalars] {off} of {9 * len(table)} floats are not bit-equal to the host's")
    assert not bad, "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------ 2. kernel cells
SEGS = [(1, 0), (3, 0), (4, 0), (5, 0), (8191, 0), (8192, 0), (8193, 0), (20, None), (8193, 1)]      # (elements, gradient offset in floats | None = null)
PRESET = [0, 6, 999, 99999, 0, 6, 999, 99999, 6]                                                     # seg_step before the launch


def _cell_case(hyper):
    steps = [s + (goff is not None) for s, (_, goff) in zip(PRESET, SEGS)]
    return dict(kind="seg", chunk=CHUNK, segs=SEGS, hyper=hyper, step=max(steps), gscale=1.0, state="rand", bias=steps, bucket=False, flatten=False, mask=None)


def _cell_inputs(case, seed):
    """The input distribution of adamw_cells.make_inputs (random starting moments), from a seed of this file."""
    N = A.n_elems(case)
    gen = torch.Generator().manual_seed(seed)
    rand = lambda: torch.rand(N, generator=gen, dtype=torch.float64)
    randn = lambda: torch.randn(N, generator=gen, dtype=torch.float64)
    mag = lambda: 10.0 ** torch.randint(-6, 3, (N,), generator=gen).double()
    g = mag() * (1 + 9 * rand()) * torch.where(rand() < 0.5, -1.0, 1.0) * (rand() >= 0.05)
    cls = torch.arange(N) % 3
    p = randn() * torch.where(cls == 0, 0.0, torch.where(cls == 1, 1e-3, 1.0))
    scale = mag()
    return dict(p=p.float(), g=g.float(), m=(randn() * scale).float(), v=(scale * scale * (0.5 + rand())).float())


def _launch_cells(lib, case, inp, lay, only_step=None):
    """One launch over the row's segments.  only_step None: advance + step_segments_dev from PRESET; else the CLASSIC kan_adamw_step_segments at
    that step with a gradient only for the segments whose count it is.  Returns (dense p / m / v, seg_step after, findings)."""
    from convkan_amd import _lib as L
    nb = lay["n_blk"]
    pos = torch.cat([torch.arange(o, o + n) for o, n in zip(lay["seg_off"], lay["seg_n"])]).cuda()
    gap = torch.ones(nb, dtype=torch.bool, device="cuda")
    gap[pos] = False
    blk = {k: torch.full((nb + 128,), SENT_F, dtype=torch.int32, device="cuda").view(torch.float32) for k in "pmv"}
    for k in "pmv":
        blk[k][64:64 + nb][pos] = inp[k].cuda()
    stores, addr = [], []
    for i, (n, goff) in enumerate(case["segs"]):
        if goff is None or (only_step is not None and case["bias"][i] != only_step):
            addr.append(0)
            continue
        stores.append(torch.full((n + goff + 1,), 7.0, device="cuda"))
        view = stores[-1][goff:goff + n]
        view.copy_(inp["g"][lay["elem_off"][i]:lay["elem_off"][i] + n])
        assert view.data_ptr() & 15 == 4 * goff
        addr.append(view.data_ptr())
    dev = lambda xs, dt: torch.tensor(xs, dtype=dt, device="cuda")
    tab = dict(seg_grad=dev(addr, torch.int64), seg_off=dev(lay["seg_off"], torch.int64), seg_n=dev(lay["seg_n"], torch.int32),
               chunk_seg=dev(lay["chunk_seg"], torch.int32), chunk_start=dev(lay["chunk_start"], torch.int32))
    seg_step = dev(PRESET, torch.int32)
    lr, (b1, b2), eps, wd = A.HYPER[case["hyper"]]
    lr_dev = torch.full((1,), lr, dtype=torch.float64, device="cuda")
    before = {k: t.clone() for k, t in tab.items()}
    stores0 = [s.clone() for s in stores]
    views = [_p(blk[k][64:64 + nb]) for k in "pmv"]
    tabs = [_p(tab[k]) for k in ("seg_grad", "seg_off", "seg_n", "chunk_seg", "chunk_start")]
    if only_step is None:
        L.check(lib.kan_adamw_advance(_p(seg_step), _p(tab["seg_grad"]), len(addr), _stream()), "kan_adamw_advance")
        L.check(lib.kan_adamw_step_segments_dev(*views, *tabs, _p(lr_dev), _p(seg_step), len(lay["chunk_seg"]), CHUNK, b1, b2, eps, wd, 1.0, _stream()),
                "kan_adamw_step_segments_dev")
    else:
        L.check(lib.kan_adamw_step_segments(*views, *tabs, _p(None), len(lay["chunk_seg"]), CHUNK, lr, b1, b2, eps, wd, only_step, 1.0, _stream()),
                "kan_adamw_step_segments")
    torch.cuda.synchronize()
    bad, out = [], {}
    for k in "pmv":
        raw = blk[k].view(torch.int32)
        if not (bool((raw[:64] == SENT_F).all()) and bool((raw[-64:] == SENT_F).all())):
            bad.append(f"{k}: memory next to the block was written")
        if not bool((raw[64:64 + nb][gap] == SENT_F).all()):
            bad.append(f"{k}: elements in the gaps between segments were written")
        out[k] = blk[k][64:64 + nb][pos].cpu()
    bad += [f"table {k} was written" for k, t in tab.items() if not torch.equal(t, before[k])]
    if not all(torch.equal(s.view(torch.int32), s0.view(torch.int32)) for s, s0 in zip(stores, stores0)):
        bad.append("a gradient buffer was written")
    if float(lr_dev[0]) != lr:
        bad.append("lr_dev was written")
    return out, seg_step.tolist(), bad


@pytest.mark.parametrize("hyper", list(A.HYPER))
def test_kernel_cells_vs_fp64_and_vs_the_classic_step(hyper, gpu_lib):
    case = _cell_case(hyper)
    lay = A.layout(case)
    inp = _cell_inputs(case, 4100 + list(A.HYPER).index(hyper))
    r64, r32 = A.reference(case, inp, torch.float64), A.reference(case, inp, torch.float32)
    got, steps, bad = _launch_cells(gpu_lib, case, inp, lay)
    lines, wrong = A.judge(case, inp, got, r64, r32)
    print(f"[capturable cells] {hyper}: " + "; ".join(lines))
    bad += wrong
    assert steps == case["bias"], (steps, case["bias"])                   # +1 wherever there is a gradient, the null segment's count unchanged
    for i, (n, goff) in enumerate(SEGS):
        sl = slice(lay["elem_off"][i], lay["elem_off"][i] + n)
        if goff is None:
            for k in "pmv":
                if not torch.equal(got[k][sl].view(torch.int32), inp[k][sl].view(torch.int32)):
                    bad.append(f"{k}: segment {i} has a null gradient and changed")
    # bit for bit the classic path wherever the nine floats agree bit for bit
    table, compared = _scalar_table(), 0
    for st in sorted(set(case["bias"][i] for i, (_, goff) in enumerate(SEGS) if goff is not None)):
        dev9, host9 = table[(hyper, st)]
        if not np.array_equal(dev9.view(np.int32), host9.view(np.int32)):
            continue
        classic, _, bad_c = _launch_cells(gpu_lib, case, inp, lay, only_step=st)
        bad += [b + f" (classic launch, step {st})" for b in bad_c]
        for i, (n, goff) in enumerate(SEGS):
            if goff is None or case["bias"][i] != st:
                continue
            compared += 1
            sl = slice(lay["elem_off"][i], lay["elem_off"][i] + n)
            for k in "pmv":
                diff = int((got[k][sl].view(torch.int32) != classic[k][sl].view(torch.int32)).sum())
                if diff:
                    bad.append(f"{k}: segment {i} (step {st}) differs from kan_adamw_step_segments in {diff} of {n} elements")
    print(f"[capturable cells] {hyper}: {compared} of {len(SEGS) - 1} segments compared bit for bit with the classic step")
    assert not bad, f"{hyper}:\n  " + "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------ 3. kan_set_u64_table
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_set_u64_table(n, gpu_lib):
    from convkan_amd import _lib as L
    sent = 0x5A5A5A5A5A5A5A5A
    first0 = 3
    table = torch.full((first0 + n + 70,), sent, dtype=torch.int64, device="cuda")
    want = [(0x7F00_0000_0000 + 0x1_0000_0001 * (i + 1)) for i in range(n)]                              # above 2^32: both halves matter
    for first in range(0, n, 64):
        part = want[first:first + 64]
        vals = (C.c_ulonglong * 64)(*part)
        L.check(gpu_lib.kan_set_u64_table(_p(table), first0 + first, vals, len(part), _stream()), "kan_set_u64_table")
        for i in range(64):
            vals[i] = 0                                                                                  # the launch carried the values
    torch.cuda.synchronize()
    got = table.tolist()
    assert got[first0:first0 + n] == want
    assert all(x == sent for x in got[:first0] + got[first0 + n:])


# ------------------------------------------------------------------------------------------------ trajectories
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
    print(f"[capturable trajectory] {tag}: " + "; ".join(line))
    return bad


def _state(opt, i, like):
    st = opt.state_dict()["state"]
    if i not in st:
        return torch.zeros_like(like), torch.zeros_like(like), 0
    return st[i]["exp_avg"], st[i]["exp_avg_sq"], int(st[i]["step"])


def _grad_list(gen, shapes, steps, late=2, late_from=3):
    """Per step one gradient per parameter (1e-3 .. 1e1 per element); parameter `late` has none before step `late_from`."""
    mk = lambda s: torch.randn(s, generator=gen) * 10.0 ** torch.randint(-3, 1, s, generator=gen).float()
    return [[None if (i == late and it < late_from) else mk(s) for i, s in enumerate(shapes)] for it in range(steps)]


def _feed(ps, opt, grads, cast, sch=None, every=3, it0=0):
    for it, step in enumerate(grads, start=it0):
        for p, g in zip(ps, step):
            p.grad = None if g is None else cast(g)
        opt.step()
        if sch is not None and (it + 1) % every == 0:
            sch.step()


HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _three(p0, cls_dev, **kw):
    """(parameters, optimizer) on the GPU with `cls_dev`, and torch.optim.AdamW(foreach=False) on fp64 and fp32 CPU copies."""
    dev = [nn.Parameter(v.clone().cuda()) for v in p0]
    r64 = [nn.Parameter(v.double()) for v in p0]
    r32 = [nn.Parameter(v.clone()) for v in p0]
    return ((dev, cls_dev(dev, **HYPER, **kw)), (r64, torch.optim.AdamW(r64, **HYPER, foreach=False)), (r32, torch.optim.AdamW(r32, **HYPER, foreach=False)))


def _start_values():
    return [(p.detach().clone() * (torch.arange(p.numel()).reshape(p.shape) % 3 != 0)).float() for p in _net().parameters()]       # every third starts at 0


def test_trajectory_with_scheduler_and_a_late_parameter(gpu_lib):
    """12 eager capturable steps, ExponentialLR(0.8) stepped every 3; parameter 2 (the PReLU slope) has a gradient from step 4 on only."""
    from convkan_amd import FusedAdamW
    p0 = _start_values()
    gen = torch.Generator().manual_seed(31)
    grads = _grad_list(gen, [tuple(v.shape) for v in p0], 12)
    (dev, opt), (r64, opt64), (r32, opt32) = _three(p0, FusedAdamW, capturable=True)
    for ps, o, cast in ((dev, opt, lambda g: g.cuda()), (r64, opt64, torch.Tensor.double), (r32, opt32, torch.Tensor.clone)):
        _feed(ps, o, grads, cast, torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.8))
    assert opt._flat[0]["tab"]["seg_step"].tolist() == [12, 12, 9, 12]
    assert abs(float(opt._flat[0]["lr_dev"][0]) - opt64.param_groups[0]["lr"] / 0.8) < 1e-15      # the lr the 12th step used: one scheduler step back
    bad = []
    for i in range(4):
        bad += _judge_trajectory(f"param {i}", p0[i], (dev[i], *_state(opt, i, dev[i])[:2]), (r64[i], *_state(opt64, i, r64[i])[:2]),
                                 (r32[i], *_state(opt32, i, r32[i])[:2]))
        assert _state(opt, i, dev[i])[2] == _state(opt64, i, r64[i])[2] == (9 if i == 2 else 12)
    assert opt.param_groups[0]["step"] == 12 and opt._flat[0]["steps"] == [12, 12, 9, 12]          # the host view, read by state_dict()
    assert not bad, "\n  ".join(bad)


def test_resume_in_every_direction(gpu_lib):
    """3 capturable steps; state_dict() into torch.optim.AdamW (fp32 CPU), into a classic FusedAdamW, and from each of those back into a fresh
    capturable one; 2 further steps everywhere end where an uninterrupted fp64 run ends; step counts exact."""
    from convkan_amd import FusedAdamW
    p0 = _start_values()
    gen = torch.Generator().manual_seed(32)
    grads = _grad_list(gen, [tuple(v.shape) for v in p0], 5, late_from=2)
    (dev, opt), (r64, opt64), (r32, opt32) = _three(p0, FusedAdamW, capturable=True)
    _feed(r64, opt64, grads, torch.Tensor.double)
    _feed(r32, opt32, grads, torch.Tensor.clone)
    cuda = lambda g: g.cuda()
    _feed(dev, opt, grads[:3], cuda)
    sd = copy.deepcopy(opt.state_dict())
    assert [int(sd["state"][i]["step"]) for i in range(4)] == [3, 3, 1, 3]
    snap = [p.detach().clone() for p in dev]

    def fresh(cls, where, **kw):
        ps = [nn.Parameter(where(v)) for v in snap]
        o = cls(ps, lr=0.5, betas=(0.1, 0.1), weight_decay=0.0, **kw)      # every hyper-parameter comes from the loaded state
        return ps, o
    runs = {"capturable throughout": (dev, opt, cuda)}
    t_ps, t_opt = fresh(torch.optim.AdamW, lambda v: v.cpu().clone(), foreach=False)
    t_opt.load_state_dict(copy.deepcopy(sd))
    runs["capturable -> torch"] = (t_ps, t_opt, torch.Tensor.clone)
    c_ps, c_opt = fresh(FusedAdamW, torch.Tensor.clone)
    c_opt.load_state_dict(copy.deepcopy(sd))
    assert c_opt._flat[0]["steps"] == [3, 3, 1, 3]
    runs["capturable -> classic"] = (c_ps, c_opt, cuda)
    for tag, src in (("torch -> capturable", t_opt), ("classic -> capturable", c_opt)):
        b_ps, b_opt = fresh(FusedAdamW, torch.Tensor.clone, capturable=True)
        b_opt.load_state_dict(copy.deepcopy(src.state_dict()))
        assert b_opt._flat[0]["tab"]["seg_step"].tolist() == [3, 3, 1, 3] and b_opt.param_groups[0]["lr"] == HYPER["lr"]
        runs[tag] = (b_ps, b_opt, cuda)
    bad = []
    for tag, (ps, o, cast) in runs.items():
        _feed(ps, o, grads[3:], cast)
        for i in range(4):
            bad += _judge_trajectory(f"{tag}, param {i}", p0[i], (ps[i], *_state(o, i, ps[i])[:2]), (r64[i], *_state(opt64, i, r64[i])[:2]),
                                     (r32[i], *_state(opt32, i, r32[i])[:2]))
            assert _state(o, i, ps[i])[2] == _state(opt64, i, r64[i])[2] == (3 if i == 2 else 5), (tag, i)
    assert not bad, "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------ 6. recorded step == eager step
SLOPE_GRAD_NOISE = 2.8e-6          # the PReLU-slope gradients "summed by atomics, differ: <= 2.8e-6 max-normalised, as between two runs"


@pytest.mark.parametrize("kind", ["KAN", "ChebyKAN"])
def test_recorded_step_with_optimizer_equals_eager_steps_bitwise(kind, gpu_lib):
    """Six steps at bs 4, eager train_step against GraphedStep(optimizer=...) from a deep copy: the six losses, every parameter, and exp_avg /
    exp_avg_sq are torch.equal; seg_step is 6 everywhere; an eager eval forward afterwards is torch.equal (the version-counter bump).

    One class of moments cannot be compared with torch.equal, on this commit or its parent: the gradient of a PReLU slope is a sum of
    per-workgroup partials added with float atomics (k_in_prelu_bwd), so two EAGER runs of these very steps already
    differ in it -- measured here, eager against eager: |dg| up to 1.5e-8, exp_avg of three slopes differing by 1e-11 .. 5e-10, exp_avg_sq by
    2e-14 .. 2e-12, no parameter differing.  For those one-element tensors (8 in KAN-VGG11) exp_avg and exp_avg_sq are bounded instead: exp_avg is a
    combination sum_k w_k g_k of the six gradients with sum |w_k| <= 1, so it moves by at most SLOPE_GRAD_NOISE x max_k |g_k|, and exp_avg_sq
    (the same with g_k^2) by at most 2 x SLOPE_GRAD_NOISE x max_k g_k^2; SLOPE_GRAD_NOISE is the project's recorded run-to-run figure.  Every
    other tensor -- all weights and biases, 99.9999 % of the elements -- and the slopes themselves are compared bit for bit."""
    import convkan_amd as K
    from convkan_amd.models import vggkan
    torch.manual_seed(7)
    base = vggkan(3, 10, arch="VGG11", kan_conv=kind, dropout_linear=0.0).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(4, 3, 32, 32, device="cuda", generator=g), torch.randint(0, 10, (4,), device="cuda", generator=g)) for _ in range(6)]
    probe = torch.randn(4, 3, 32, 32, device="cuda", generator=g)
    out, gmax = {}, {}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base)
        slopes = {i for i, (n, p) in enumerate(model.named_parameters()) if isinstance(model.get_submodule(n.rsplit(".", 1)[0]), nn.PReLU)}
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        params = opt._flat[0]["params"]
        with torch.no_grad():
            model.eval()
            model(probe)                                # an eager forward BEFORE training: the packed-weight cache now holds the initial weights
            model.train()
        losses = []
        if mode == "eager":
            for d, t in batches:
                losses.append(K.train_step(model, d, t, opt).clone())
                for i in slopes:
                    gmax[i] = torch.maximum(gmax.get(i, torch.zeros((), device="cuda")), params[i].grad.abs().max())
        else:
            step = K.GraphedStep(model, batches[0][0], batches[0][1], optimizer=opt)
            assert opt._flat[0]["tab"]["seg_step"].tolist() == [0] * len(params)      # the warm-up was undone
            losses = [step(d, t).clone() for d, t in batches]
        torch.cuda.synchronize()
        flat = opt._flat[0]
        with torch.no_grad():
            model.eval()
            y = model(probe).clone()                    # an eager forward AFTER: must see the weights the replays wrote (version counters)
        out[mode] = ([float(x) for x in losses], [tuple(t.clone() for t in v) for v in flat["views"]], flat["tab"]["seg_step"].tolist(), y)
    e, r = out["eager"], out["graph"]
    assert all(e[1][i][0].numel() == 1 for i in slopes) and (len(slopes) == 8 or kind != "KAN")
    assert e[0] == r[0], (e[0], r[0])
    assert e[0][0] != e[0][-1]
    assert e[2] == r[2] == [6] * len(e[2])
    bad = []
    for i, (a, b) in enumerate(zip(e[1], r[1])):
        if not torch.equal(a[0], b[0]):
            bad.append(f"parameter {i}: {int((a[0] != b[0]).sum())} elements differ")
        for row, name, width in ((1, "exp_avg", 1.0), (2, "exp_avg_sq", 2.0)):
            if i in slopes:
                d, tol = float((a[row].double() - b[row].double()).abs().max()), width * SLOPE_GRAD_NOISE * float(gmax[i]) ** row
                print(f"[capturable graph] {kind} slope {i} {name}: |eager - recorded| {d:.2e} (bound {tol:.2e}, max |g| {float(gmax[i]):.2e})")
                if not d <= tol:
                    bad.append(f"{name} of slope {i}: {d:.3e} > {tol:.3e}")
            elif not torch.equal(a[row], b[row]):
                bad.append(f"{name} of parameter {i}: {int((a[row] != b[row]).sum())} elements differ")
    assert not bad, "\n  ".join(bad)
    assert torch.equal(e[3], r[3])


# ------------------------------------------------------------------------------------------------ 7. scheduler through the graph
def _small_batches(n, sizes):
    g = torch.Generator(device="cuda").manual_seed(5)
    return [(torch.randn(b, 7, device="cuda", generator=g), torch.randint(0, 3, (b,), device="cuda", generator=g)) for b in sizes[:n]]


def test_scheduler_moves_lr_between_replays(gpu_lib):
    import convkan_amd as K
    batches = _small_batches(6, [8] * 6)
    out = {}
    for mode in ("eager", "graph"):
        model = _net().cuda().train()
        opt = K.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, capturable=True)
        sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.8)
        step = K.GraphedStep(model, *batches[0], optimizer=opt) if mode == "graph" else None
        losses = []
        for it, (d, t) in enumerate(batches):
            losses.append(float(step(d, t) if step is not None else K.train_step(model, d, t, opt)))
            if it == 2:
                sch.step()
        torch.cuda.synchronize()
        out[mode] = (losses, opt._flat[0]["block"].clone(), float(opt._flat[0]["lr_dev"][0]), opt._flat[0]["tab"]["seg_step"].tolist())
    assert out["eager"][0] == out["graph"][0]
    assert torch.equal(out["eager"][1], out["graph"][1])
    assert out["eager"][2] == out["graph"][2] == 1e-2 * 0.8
    assert out["eager"][3] == out["graph"][3] == [6, 6, 6, 6]


def test_recording_with_a_stale_lr_raises(gpu_lib):
    import convkan_amd as K
    from convkan_amd._lib import KanConvError
    model = _net().cuda().train()
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, capturable=True)
    d, t = _small_batches(1, [8])[0]
    K.train_step(model, d, t, opt)                       # lr is on the device now
    before = opt._flat[0]["block"].clone()
    opt.param_groups[0]["lr"] = 5e-3                     # ... and stale now
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
    assert float(opt._flat[0]["lr_dev"][0]) == 5e-3


# ------------------------------------------------------------------------------------------------ 8. drivers
def test_graphed_driver_equals_the_eager_loop(gpu_lib):
    """Three batches of 8 and a ragged fourth of 5, two epochs: the graphed driver replays the first three and sends the fourth through eager
    train_step; its per-epoch losses are those of an eager loop over a capturable optimizer, to the last bit."""
    import convkan_amd as K
    from convkan_amd import train as T
    batches = _small_batches(4, [8, 8, 8, 5])
    got = T.train_model_generic(_net(), batches, device="cuda", learning_rate=1e-2, weight_decay=1e-2, gamma=0.8, epochs=2, graphed=True)
    model = _net().cuda().train()
    opt = K.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, capturable=True)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.8)
    want = []
    for _ in range(2):
        total = torch.zeros((), device="cuda")
        for d, t in batches:
            total += K.train_step(model, d, t, opt, nn.CrossEntropyLoss())
        want.append(float(total) / 4)
        sch.step()
    assert got == want and got[0] != got[1], (got, want)
    assert opt._flat[0]["tab"]["seg_step"].tolist() == [8, 8, 8, 8]


def test_graphed_train_and_test_models_equals_the_eager_one(gpu_lib):
    """The same batches through train_and_test_models twice, eager and graphed, each with its own capturable optimizer and scheduler: all seven
    returned lists are equal -- the evaluation after every epoch reads the weights the replays wrote."""
    import convkan_amd as K
    from convkan_amd import train as T
    batches, tests = _small_batches(4, [8, 8, 8, 5]), _small_batches(2, [8, 8])
    out = []
    for graphed in (False, True):
        model = _net().cuda()
        opt = K.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, capturable=True)
        sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.8)
        out.append(T.train_and_test_models(model, batches, tests, opt, sch, epochs=2, graphed=graphed))
        assert opt._flat[0]["tab"]["seg_step"].tolist() == [8, 8, 8, 8]
    assert out[0] == out[1], out
    assert out[0][0][0] != out[0][0][1] and out[0][6] == [1e-2, 1e-2 * 0.8]
