"""FusedAdamW: host layout logic on CPU; the fused step against torch.optim.AdamW -- the optimizer
the reference builds (generic_train.py:24) -- on the GPU: a short fp32 comparison, then trajectories against fp64 CPU copies (groups,
add_param_group, ExponentialLR, every gradient form step() accepts, resume through state_dict in both directions).  The kernels' own launch
cells: tests/test_gpu_adamw_matrix.py."""
import copy

import pytest
import torch
import torch.nn as nn

import convkan_amd as K
from convkan_amd import _lib as L


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 5), nn.PReLU(), nn.Linear(5, 3, bias=False))


def test_flat_layout_and_views():
    net = _net()
    before = [p.detach().clone() for p in net.parameters()]
    opt = K.FusedAdamW(net.parameters(), lr=1e-3, weight_decay=1e-4)
    flat = opt._flat[0]
    assert flat["block"].shape[0] == 3 and flat["n"] % 64 == 0
    base = flat["block"].data_ptr()
    for p, b in zip(net.parameters(), before):
        assert torch.equal(p, b)                                             # values survive the move into the block
        off = p.data_ptr() - base
        assert 0 <= off < flat["n"] * 4 and off % 256 == 0                   # a 256-byte aligned view of row 0
    tab = flat["tab"]                                                        # chunk table of kan_adamw_step_segments
    sizes = [p.numel() for p in net.parameters()]
    assert tab["seg_n"].tolist() == sizes and tab["seg_off"].tolist() == [0, 64, 128, 192]
    assert tab["chunk_seg"].tolist() == [0, 1, 2, 3] and tab["chunk_start"].tolist() == [0, 0, 0, 0]
    big = K.FusedAdamW([nn.Parameter(torch.zeros(20000)), nn.Parameter(torch.zeros(5))])._flat[0]["tab"]
    assert big["chunk_seg"].tolist() == [0, 0, 0, 1] and big["chunk_start"].tolist() == [0, 8192, 16384, 0]
    net(torch.randn(2, 7)).sum().backward()
    assert all(p.grad is not None and p.grad.data_ptr() != 0 for p in net.parameters())
    opt.zero_grad()
    assert all(p.grad is None for p in net.parameters())                     # torch's own zero_grad: nothing to zero per step
    with pytest.raises(L.KanConvError, match="no CPU fallback"):
        net(torch.randn(2, 7)).sum().backward()
        opt.step()


def test_scheduler_and_state_dict_surface():
    net = _net()
    opt = K.FusedAdamW(net.parameters(), lr=1e-3, weight_decay=1e-4)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.8)
    sch.step()
    assert abs(opt.param_groups[0]["lr"] - 8e-4) < 1e-12
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["exp_avg"].shape == (5, 7)
    ref = torch.optim.AdamW(_net().parameters(), lr=1e-3, weight_decay=1e-4)
    assert len(sd["state"]) == len(list(net.parameters())) and set(sd["param_groups"][0]) >= set(ref.state_dict()["param_groups"][0]) - {
        "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"}
    sd2 = copy.deepcopy(sd)
    sd2["state"][0]["exp_avg"].fill_(0.5); sd2["state"][0]["step"] = torch.tensor(7.0)
    opt.load_state_dict(sd2)
    assert float(opt._flat[0]["views"][0][1].mean()) == 0.5 and opt.param_groups[0]["step"] == 7
    with pytest.raises(ValueError):
        K.FusedAdamW(_net().parameters(), lr=-1.0)


@pytest.mark.gpu
def test_fused_step_matches_torch_adamw(gpu_lib):
    """Six steps with a decaying learning rate on identical gradients; a parameter without gradient is skipped as torch skips
    it, and bias-corrected with its own step count once its gradients arrive."""
    net = _net()
    ref = copy.deepcopy(net)
    extra_h, extra_r = nn.Parameter(torch.randn(130)), None
    extra_r = nn.Parameter(extra_h.detach().clone())
    dev = net.cuda()
    extra_d = nn.Parameter(extra_h.detach().cuda())
    opt = K.FusedAdamW(list(dev.parameters()) + [extra_d], lr=1e-2, weight_decay=1e-2)
    opt_r = torch.optim.AdamW(list(ref.parameters()) + [extra_r], lr=1e-2, weight_decay=1e-2, foreach=False)
    s1, s2 = (torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.8) for o in (opt, opt_r))
    for it in range(6):
        x = torch.randn(16, 7, generator=torch.Generator().manual_seed(it))
        opt.zero_grad(); opt_r.zero_grad()
        (ref(x) ** 2).mean().backward()
        for pd, pr in zip(dev.parameters(), ref.parameters()):               # the same gradients on both sides: only the update differs
            pd.grad = pr.grad.detach().clone().cuda()
        if it >= 3:                                                          # the extra parameter only gets gradients later
            extra_d.grad = torch.full((130,), 0.1 * it).cuda(); extra_r.grad = torch.full((130,), 0.1 * it)
        else:
            extra_d.grad = None
        opt.step(); opt_r.step(); s1.step(); s2.step()
    for a, b in zip(list(dev.parameters()) + [extra_d], list(ref.parameters()) + [extra_r]):
        assert float((a.detach().cpu() - b.detach()).abs().max()) <= 2e-6 * float(b.abs().max()) + 1e-7
    sd, sr = opt.state_dict()["state"], opt_r.state_dict()["state"]
    for i in sr:
        assert float((sd[i]["exp_avg"].cpu() - sr[i]["exp_avg"]).abs().max()) <= 2e-6 * float(sr[i]["exp_avg"].abs().max()) + 1e-9
        assert float((sd[i]["exp_avg_sq"].cpu() - sr[i]["exp_avg_sq"]).abs().max()) <= 2e-6 * float(sr[i]["exp_avg_sq"].abs().max()) + 1e-12


@pytest.mark.gpu
def test_large_block_and_alignment_errors(gpu_lib):
    """A 5 M-element block (grid-stride path, ragged tail) against the closed-form first step; misaligned blocks are refused."""
    import ctypes as C
    n = 5_000_003
    g = torch.Generator(device="cuda").manual_seed(1)
    p, gr = torch.randn(n, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    p0 = p.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, o=0: C.c_void_p(t.data_ptr() + 4 * o)
    L.check(L.load().kan_adamw_step(ptr(p), ptr(gr), ptr(m), ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, st), "adamw")
    # step 1: m = 0.1 g, v = 0.001 g^2, update = lr * g / (|g| + eps)
    want = p0 * (1 - 1e-5) - 1e-3 * gr / (gr.abs() + 1e-8)
    assert float((p - want).abs().max()) < 1e-6 and float((m - 0.1 * gr).abs().max()) < 1e-6
    assert L.load().kan_adamw_step(ptr(p, 1), ptr(gr), ptr(m), ptr(v), 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, st) != 0
    assert L.load().kan_adamw_step(ptr(p), ptr(gr), ptr(m), ptr(v), 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, st) != 0


@pytest.mark.gpu
def test_train_model_generic_reduces_loss(gpu_lib):
    """The harness on a small KAN-VGG: AdamW + ExponentialLR as generic_train.py:24-25; the loss on a fixed batch drops."""
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    m = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear", dropout_linear=0.0)
    x, t = torch.randn(8, 3, 32, 32), torch.randint(0, 10, (8,))
    hist = K.train_model_generic(m, [(x, t)] * 3, device="cuda", learning_rate=1e-3, weight_decay=1e-4, gamma=0.8, epochs=4)
    assert len(hist) == 4 and hist[-1] < hist[0] and all(h == h for h in hist)


@pytest.mark.gpu
def test_packed_weights_follow_every_weight_update(gpu_lib, monkeypatch):
    """Single-group layers keep their packed weight layouts between calls (ops._PACKED).  Every way of changing the weights must
    be seen: in-place ops (version counter), FusedAdamW's raw-pointer kernel (it bumps the counters), and writes the counters
    cannot see -- `.data` ops, a raw copy into the storage -- which the device-side fingerprint catches.  The check is a
    fresh, cache-free pack of the same weights (KAN_PACK_CACHE=0 path)."""
    from convkan_amd import ops
    if ops._PACK_CACHE_MAX <= 0:
        pytest.skip("packed-weight cache disabled (KAN_PACK_CACHE=0)")
    torch.manual_seed(0)
    layer = K.KANConv2DLayer(8, 128, 3, padding=1).cuda()
    x = torch.randn(4, 8, 8, 8, device="cuda")

    def uncached():
        keep, ops._PACK_CACHE_MAX = ops._PACK_CACHE_MAX, 0
        try:
            with torch.no_grad():
                return layer(x)
        finally:
            ops._PACK_CACHE_MAX = keep
    ops._PACKED.clear()
    ops.PACK_STATS.update(calls=0, forced=0, skipped=0)
    monkeypatch.setattr(ops, "_PACK_VERIFY_EVERY", 1)                                # fingerprint on every call (cadence: last part of this test)
    with torch.no_grad():
        y0 = layer(x)
        y1 = layer(x)
    assert len(ops._PACKED) == 1 and ops.PACK_STATS == {"calls": 2, "forced": 1, "skipped": 0} and torch.equal(y0, y1) and torch.equal(y0, uncached())
    assert torch.equal(layer(x).detach(), y0)                                        # the training forward shares the layouts (+ wd: one forced pack)
    with torch.no_grad():
        layer.spline_conv[0].weight.mul_(1.5)                                        # version counter moves
        y2 = layer(x)
    assert not torch.equal(y2, y0) and torch.equal(y2, uncached())
    forced = ops.PACK_STATS["forced"]
    layer.spline_conv[0].weight.data.mul_(0.5)                                       # invisible to the version counter
    layer.base_conv[0].weight.data[3, 2, 1, 1] = 7.0                                 # a single element
    with torch.no_grad():
        y3 = layer(x)
    assert ops.PACK_STATS["forced"] == forced                                        # the host saw nothing ...
    assert not torch.equal(y3, y2) and torch.equal(y3, uncached())                   # ... the fingerprint did
    opt = K.FusedAdamW(layer.parameters(), lr=1e-2)
    with torch.no_grad():
        y4 = layer(x)                                                                # parameters now live in the optimizer's flat block
    assert torch.equal(y4, y3)
    layer(x).square().mean().backward()
    opt.step()
    with torch.no_grad():
        y5 = layer(x)
    assert not torch.equal(y5, y4) and torch.equal(y5, uncached())
    # a graph that saved the old bwd-data layout must not be differentiated after the weights moved
    out = layer(x.requires_grad_(True)).square().mean()
    with torch.no_grad():
        layer.spline_conv[0].weight.add_(0.01)
        layer(x)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward()
    # verification cadence (the default is every 16th call): a stamp-visible write re-packs at once; a raw write is seen at once after
    # ops.weights_changed(), and at the 4th call at the latest with a cadence of 4; unchanged weights cost no device work in between
    monkeypatch.setattr(ops, "_PACK_VERIFY_EVERY", 4)
    with torch.no_grad():
        ya = layer(x)
        calls, skipped = ops.PACK_STATS["calls"], ops.PACK_STATS["skipped"]
        assert torch.equal(layer(x), ya) and torch.equal(layer(x), ya)
        assert ops.PACK_STATS["calls"] == calls and ops.PACK_STATS["skipped"] == skipped + 2
        layer.spline_conv[0].weight.mul_(1.1)                                        # version counter: seen on the very next call
        yb = layer(x)
        assert not torch.equal(yb, ya) and torch.equal(yb, uncached())
        layer.spline_conv[0].weight.data.mul_(0.9)                                   # raw write ...
        ops.weights_changed()                                                        # ... announced
        yc = layer(x)
        assert not torch.equal(yc, yb) and torch.equal(yc, uncached())
        layer.spline_conv[0].weight.data.mul_(1.2)                                   # raw write, not announced: picked up within the cadence
        outs = [layer(x) for _ in range(4)]
        assert torch.equal(outs[-1], uncached()) and not torch.equal(outs[-1], yc)


# ------------------------------------------------------------------------------------------------ trajectories against fp64 torch.optim.AdamW
# FusedAdamW on the GPU against torch.optim.AdamW(foreach=False) on fp64 CPU copies fed the same gradients; the same run in fp32 on the CPU is
# the noise measure.  Judged as tests/adamw_cells.py judges a step: parameters that started at 0 and the rest, each class normalised by the fp64
# reference's largest element in it; exp_avg by the reference's largest element; exp_avg_sq elementwise relative (a sum of non-negative terms).
# Tolerance per tensor: max(2e-6, 4 x the fp32 CPU run's own error).
def _grads(gen, shape, half=False):
    """A gradient whose size varies from element to element and step to step (1e-3 .. 1e1); `half`: values an fp16 tensor holds exactly."""
    g = torch.randn(shape, generator=gen) * 10.0 ** torch.randint(-3, 1, shape, generator=gen).float()
    return g.half().float() if half else g


def _start(gen, shape):
    n = torch.Size(shape).numel()
    return (torch.randn(shape, generator=gen) * (torch.arange(n).reshape(shape) % 3 != 0)).float()          # every third element starts at 0


def _judge_trajectory(tag, p0, got, r64, r32):
    """got / r64 / r32: (p, exp_avg, exp_avg_sq).  Returns the failures."""
    from adamw_cells import FLOOR
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
        tol = max(FLOOR, 4.0 * noise[name])
        line.append(f"{name} {e:.1e} (tol {tol:.1e}, fp32 reference {noise[name]:.1e})")
        if not e <= tol:
            bad.append(f"{tag} {name}: error {e:.3e} > {tol:.3e} (fp32 reference {noise[name]:.3e})")
    print(f"[adamw trajectory] {tag}: " + "; ".join(line))
    return bad


def _state_of(opt, p):
    st = opt.state_dict()["state"]
    idx = [id(q) for g in opt.param_groups for q in g["params"]].index(id(p))
    if idx not in st:
        return torch.zeros_like(p), torch.zeros_like(p), 0
    return st[idx]["exp_avg"], st[idx]["exp_avg_sq"], int(st[idx]["step"])


def _padding_is_zero(opt):
    for flat in opt._flat:
        if flat is None:
            continue
        pad = torch.ones(flat["n"], dtype=torch.bool)
        for o, n in zip(flat["tab"]["seg_off"].tolist(), flat["tab"]["seg_n"].tolist()):
            pad[o:o + n] = False
        assert bool(pad.any()) and bool((flat["block"].cpu()[:, pad].view(torch.int32) == 0).all()), "alignment elements between parameters were written"


@pytest.mark.gpu
def test_trajectory_groups_scheduler_and_gradient_forms(gpu_lib):
    """12 steps under ExponentialLR: two groups with their own lr / betas / eps / weight_decay and a third added through add_param_group;
    a 20003-element parameter whose gradient is a view one float into a flat buffer (scalar path), a 5-element one with an fp16 gradient,
    a frozen one, one with a non-contiguous gradient that only arrives from step 4, one whose gradient moves every step and is gone from
    step 8, and a betas = (0, 0) group."""
    gen = torch.Generator().manual_seed(11)
    spec = dict(a=(20003,), b=(5,), frozen=(33,), c=(7, 9), d=(300,), e=(8195,))
    p0 = {k: _start(gen, s) for k, s in spec.items()}
    g0 = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    g1 = dict(lr=3e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.3)
    g2 = dict(lr=1e-2, betas=(0.0, 0.0), eps=1e-8, weight_decay=1e-2)

    def build(make, cls):
        ps = {k: nn.Parameter(make(v), requires_grad=k != "frozen") for k, v in p0.items()}
        opt = cls([dict(params=[ps["a"], ps["b"], ps["frozen"]], **g0), dict(params=[ps["c"], ps["d"]], **g1)])
        opt.add_param_group(dict(params=[ps["e"]], **g2))
        return ps, opt, torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.8)
    torch_adamw = lambda groups: torch.optim.AdamW(groups, foreach=False)
    dev, opt, sch = build(lambda v: v.clone().cuda(), K.FusedAdamW)
    r64, opt64, sch64 = build(lambda v: v.double(), torch_adamw)
    r32, opt32, sch32 = build(lambda v: v.clone(), torch_adamw)
    dev["b"].grad_dtype = None                                           # this parameter accepts a gradient of another dtype
    flatbuf = torch.zeros(20003 + 8, device="cuda")
    wide = torch.zeros(7, 18, device="cuda")
    moved, uploads = [], 0
    for it in range(12):
        grads = dict(a=_grads(gen, (20003,)), b=_grads(gen, (5,), half=True), frozen=None, c=_grads(gen, (7, 9)) if it >= 3 else None,
                     d=_grads(gen, (300,)) if it < 7 else None, e=_grads(gen, (8195,)))
        for ps, cast in ((r64, torch.Tensor.double), (r32, torch.Tensor.clone)):
            for k, g in grads.items():
                ps[k].grad = None if g is None else cast(g)
        flatbuf[1:20004].copy_(grads["a"])
        dev["a"].grad = flatbuf[1:20004]
        dev["b"].grad = grads["b"].half().cuda()
        if grads["c"] is not None:
            wide[:, ::2] = grads["c"].cuda()
            dev["c"].grad = wide[:, ::2]
        moved.append(grads["d"].cuda() if grads["d"] is not None else None)          # (kept alive: every step's gradient has a new address)
        dev["d"].grad = moved[-1]
        dev["e"].grad = grads["e"].cuda()
        if it == 0:
            assert dev["a"].grad.data_ptr() & 15 == 4 and dev["b"].grad.dtype == torch.float16
        if it == 3:
            assert not dev["c"].grad.is_contiguous()
        before = opt._flat[1]["tab"]["grad_ptrs"]
        for o, s in ((opt, sch), (opt64, sch64), (opt32, sch32)):
            o.step(); s.step()
        uploads += opt._flat[1]["tab"]["grad_ptrs"] != before
    assert uploads >= 8, "group 1's address table is re-uploaded on every step until d's gradient is gone, and once after"
    assert len({m.data_ptr() for m in moved if m is not None}) == 7
    bad = []
    for k in spec:
        got = (dev[k], *_state_of(opt, dev[k])[:2])
        bad += _judge_trajectory(k, p0[k], got, (r64[k], *_state_of(opt64, r64[k])[:2]), (r32[k], *_state_of(opt32, r32[k])[:2]))
        assert _state_of(opt, dev[k])[2] == _state_of(opt64, r64[k])[2] == dict(a=12, b=12, frozen=0, c=9, d=7, e=12)[k], k
    assert torch.equal(dev["frozen"].cpu(), p0["frozen"])
    assert [abs(g["lr"] - h["lr"]) < 1e-15 for g, h in zip(opt.param_groups, opt64.param_groups)] == [True] * 3
    _padding_is_zero(opt)
    assert not bad, "\n  ".join(bad)


def _resume_setup(seed):
    gen = torch.Generator().manual_seed(seed)
    spec = dict(w=(20003,), late=(64,), s=(5,))
    p0 = {k: _start(gen, s) for k, s in spec.items()}
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    grads = [dict(w=_grads(gen, (20003,)), late=_grads(gen, (64,)) if it >= 2 else None, s=_grads(gen, (5,))) for it in range(8)]
    return spec, p0, hyper, grads


def _feed(ps, opt, grads, cast):
    for step in grads:
        for k, g in step.items():
            ps[k].grad = None if g is None else cast(g)
        opt.step()


@pytest.mark.gpu
def test_resume_from_fused_into_torch_adamw(gpu_lib):
    """4 fused steps, state_dict() into a fresh torch.optim.AdamW, 4 more on both sides: both end where an uninterrupted fp64 run ends."""
    spec, p0, hyper, grads = _resume_setup(21)
    make = lambda cast, cls, **kw: (lambda ps: (ps, cls(list(ps.values()), **hyper, **kw)))({k: nn.Parameter(cast(v)) for k, v in p0.items()})
    r64, opt64 = make(torch.Tensor.double, torch.optim.AdamW, foreach=False)
    r32, opt32 = make(torch.Tensor.clone, torch.optim.AdamW, foreach=False)
    dev, opt = make(lambda v: v.clone().cuda(), K.FusedAdamW)
    _feed(r64, opt64, grads, torch.Tensor.double)
    _feed(r32, opt32, grads, torch.Tensor.clone)
    _feed(dev, opt, grads[:4], lambda g: g.cuda())
    sd = opt.state_dict()
    assert [int(sd["state"][i]["step"]) for i in range(3)] == [4, 2, 4]
    cont = {k: nn.Parameter(dev[k].detach().cpu().clone()) for k in spec}
    opt_c = torch.optim.AdamW(list(cont.values()), foreach=False)
    opt_c.load_state_dict(copy.deepcopy(sd))
    _feed(cont, opt_c, grads[4:], torch.Tensor.clone)
    _feed(dev, opt, grads[4:], lambda g: g.cuda())
    bad = []
    for k in spec:
        ref = (r64[k], *_state_of(opt64, r64[k])[:2])
        noise = (r32[k], *_state_of(opt32, r32[k])[:2])
        bad += _judge_trajectory(k + " (fused throughout)", p0[k], (dev[k], *_state_of(opt, dev[k])[:2]), ref, noise)
        bad += _judge_trajectory(k + " (torch after 4 fused steps)", p0[k], (cont[k], *_state_of(opt_c, cont[k])[:2]), ref, noise)
        assert _state_of(opt_c, cont[k])[2] == _state_of(opt, dev[k])[2] == _state_of(opt64, r64[k])[2]
    _padding_is_zero(opt)
    assert not bad, "\n  ".join(bad)


@pytest.mark.gpu
def test_resume_from_torch_adamw_into_fused(gpu_lib):
    """4 steps of torch.optim.AdamW (one parameter has 2: per-parameter step counts differ), its state_dict() into a fresh FusedAdamW, 4 more."""
    spec, p0, hyper, grads = _resume_setup(22)
    make = lambda cast, **kw: (lambda ps: (ps, torch.optim.AdamW(list(ps.values()), **hyper, foreach=False)))({k: nn.Parameter(cast(v)) for k, v in p0.items()})
    r64, opt64 = make(torch.Tensor.double)
    r32, opt32 = make(torch.Tensor.clone)
    _feed(r64, opt64, grads, torch.Tensor.double)
    _feed(r32, opt32, grads[:4], torch.Tensor.clone)
    sd = copy.deepcopy(opt32.state_dict())
    assert [int(sd["state"][i]["step"]) for i in range(3)] == [4, 2, 4]
    dev = {k: nn.Parameter(r32[k].detach().clone().cuda()) for k in spec}
    opt = K.FusedAdamW(list(dev.values()), lr=0.5, betas=(0.1, 0.1), weight_decay=0.0)          # every hyper-parameter comes from the loaded state
    opt.load_state_dict(sd)
    assert opt._flat[0]["steps"] == [4, 2, 4] and opt.param_groups[0]["lr"] == hyper["lr"] and tuple(opt.param_groups[0]["betas"]) == hyper["betas"]
    _feed(r32, opt32, grads[4:], torch.Tensor.clone)
    _feed(dev, opt, grads[4:], lambda g: g.cuda())
    bad = []
    for k in spec:
        bad += _judge_trajectory(k, p0[k], (dev[k], *_state_of(opt, dev[k])[:2]), (r64[k], *_state_of(opt64, r64[k])[:2]),
                                 (r32[k], *_state_of(opt32, r32[k])[:2]))
        assert _state_of(opt, dev[k])[2] == _state_of(opt64, r64[k])[2] == 8 - 2 * (k == "late")
    _padding_is_zero(opt)
    assert not bad, "\n  ".join(bad)
